"""
conv32_skip_emul on the CPU: (1) with every rounding switched off it IS the fp64 ResBlock tail
F.conv3d(silu(A h + B), w2) + F.conv3d(x, w1) + biases; (2) the bar test_gpu_conv32_skip.py holds the fused kernel to
(test_gpu_conv32.py's E_acc + silu with the fused accumulator's length) sees the plausible bugs of the fused form --
x staged without its lo halves, x staged at the Winograd-D gain, rho left out -- by at least 10x, on the geometries and
magnitudes that test runs.
"""

import functools

import pytest
import torch
import torch.nn.functional as F

import conv32_skip_emul as S

U = 2.0 ** -24


make = S.skip_inputs
emul = S.emulate


@functools.lru_cache(maxsize=None)
def _case(name):
    """(inputs, the emulation of the kernel's arithmetic), computed once per case"""
    t = make(**CASES[name])
    return t, emul(t)


def bar(t, em, split=1):
    """test_gpu_conv32.elem_bound with the fused accumulator's m = 3 (9 CinPad_h + CinPad_x) + S + 8 (+ 16 if split)"""
    ch, cx = t["h"][0].shape[1], sum(x.shape[1] for x in t["xs"])
    m = 3 * (9 * ch + cx) + split + 8 + (16 if split > 1 else 0)
    return 8.0 * U * torch.sqrt(m * em["sqterms"] / 3.0) + 2 * U * (em["trabs"] + em["out"].abs()) + em["silu"]


SMALL = dict(D=3, H=8, W=8, Ch=32)
CASES = {
    "one": dict(**SMALL),
    "concat": dict(Cx=(32, 32), **SMALL),
    "h_small_x_large": dict(N=2, mags=((1e-6, 1.0), (1.0, 1e-6)), **SMALL),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_emulation_is_the_fp64_resblock_tail(name):
    t, em = _case(name)
    A, B = (a.double()[:, :, None, None, None] for a in t["aff"])
    ref = (F.conv3d(F.silu(t["h"][0].double() * A + B), t["w2"].double(), padding=1)
           + F.conv3d(torch.cat(t["xs"], 1).double(), t["w1"].double())
           + (t["b2"].double() + t["b1"].double()).reshape(1, -1, 1, 1, 1))
    got = emul(t, exact=True)["out"]
    assert (got - ref).abs().max() <= 1e-12 * ref.abs().max()
    # and the rounded emulation is fp32-grade against it
    top = ref.abs().amax(dim=(2, 3, 4), keepdim=True)
    assert ((em["out"] - ref).abs() <= 16 * U * top + em["silu"]).all()


def test_composed_record_is_the_two_launches():
    """conv32_skip_emul.composed (from the fused record's pieces) is conv32_emul.conv32 called launch by launch"""
    import conv32_emul as E
    t, em = _case("concat")
    c1, c2 = S.composed(em, t["b2"], t["b1"])
    d1 = E.conv32(t["xs"], t["w1"], t["b1"], 1, bound=t["bound_x"])
    d2 = E.conv32(t["h"], t["w2"], t["b2"], 3, aff=t["aff"], act=True, bound=t["bound_h"], res=d1["stored"].float(),
                  res_mode="same")
    for got, want in ((c1, d1), (c2, d2)):
        for key in ("out", "stored", "absterms", "sqterms", "trabs", "silu"):
            assert torch.equal(got[key], want[key]), key


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("mutation", [dict(drop_x_lo=True), dict(sx_gain=2.0), dict(use_rho=False)],
                         ids=["drop_x_lo", "sx_gain_2", "no_rho"])
def test_bar_sees_the_plausible_bugs(name, mutation):
    t, em = _case(name)
    B = bar(t, em)
    bad = emul(t, **mutation)
    ratio = ((bad["out"] - em["out"]).abs() / B).amax(dim=(1, 2, 3, 4))
    print(name, mutation, [float(r) for r in ratio])
    if mutation.get("use_rho") is False:
        # rho = 1 for a sample whose two units coincide: the bug shows where they differ, by orders of magnitude
        e2, e1 = em["parts"]
        differs = [e2["S"][n] != e1["S"][n] or not torch.equal(e2["wscale"], e1["wscale"]) for n in range(len(ratio))]
        assert any(differs)
        assert all(float(ratio[n]) >= 10.0 for n in range(len(ratio)) if differs[n])
    else:
        # the x term must carry weight in the sample for the bug to show: every sample but one whose x is 1e-6 of h
        mags = CASES[name].get("mags", ((1.0, 1.0),))
        for n, (hm, xm) in enumerate(mags):
            if xm >= hm:
                assert float(ratio[n]) >= 10.0, (n, float(ratio[n]))
