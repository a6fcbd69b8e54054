"""
The packed weight images, byte for byte, against pack_ref.py.

Every operation of the packers is specified to the bit -- an exact maximum, one correctly rounded fp32 divide,
floor(log2), exact power-of-two products, single-rounded fp32 adds in the transforms, RNE conversions -- so the
comparison is torch.equal on the bytes.  The one input condition that makes this fair (log2 of the scale's quotient
at least 2^-10 from an integer) is asserted by pack_ref.weights on the CPU (test_pack_ref_cpu.py runs it without a
GPU).  Every input carries the four special couts of pack_ref.SPECIAL: all-zero (scale 1), largest weight 1e-30
(clamp 2^24), 1e10 (clamp 2^-24) and 3.2e38 (the m < 3e38 branch: scale 1).

Shapes: (5, 3) pads both cout and ci inside one block; (40, 24) has a partly filled second 16-channel block and a
cout pad past one 32; the Winograd-D and phase forms exist for Cout % 128 == 0, Cin % 16 == 0: one and two chunks.
"""

import functools

import pytest
import torch

import pack_ref as R

pytestmark = pytest.mark.gpu

PLAIN = [(5, 3), (40, 24)]
WZ = [(128, 16), (128, 32)]


@functools.lru_cache(maxsize=None)
def weights(Cout, Cin, k):
    return R.case_weights(Cout, Cin, k)


@functools.lru_cache(maxsize=None)
def reference(Cout, Cin, k, precision):
    return R.image(weights(Cout, Cin, k), 1 if precision == 2 else 3 if precision == 4 else precision)


@pytest.fixture(scope="module")
def hc():
    import hipcall
    return hipcall


def check_scales(got, Cout, Cin, taps):
    """the special couts' scales (fp32 1 / s behind the taps), read from the device image itself"""
    CoutPad, CinPad = R.pads(Cout, Cin)
    body = taps * CinPad * CoutPad * 4
    ws = got[body:body + CoutPad * 4].view(torch.float32)
    for c, s in R.SPECIAL_SCALE.items():
        assert ws[c].item() == 1.0 / s, (c, ws[c].item())
    assert (ws[Cout:] == 1.0).all()


@pytest.mark.parametrize("precision", [0, 1, 2, 5])
@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("Cout,Cin", PLAIN)
def test_plain_image(hc, Cout, Cin, k, precision):
    got = hc.pack(weights(Cout, Cin, k).cuda(), precision).cpu()
    ref = reference(Cout, Cin, k, precision)
    assert got.numel() == ref.numel()
    pad = R.padding(Cout, Cin, k ** 3, precision)
    assert pad.any() and (got[:pad.numel()][pad] == 0).all()
    assert torch.equal(got, ref)
    if precision in (1, 2):
        check_scales(got, Cout, Cin, k ** 3)


@pytest.mark.parametrize("k", [3, 1])
@pytest.mark.parametrize("Cout,Cin", PLAIN)
def test_precisions_1_and_2_share_the_image(hc, Cout, Cin, k):
    w = weights(Cout, Cin, k).cuda()
    assert torch.equal(hc.pack(w, 1), hc.pack(w, 2))


@pytest.mark.parametrize("precision", [3, 4, 6])
@pytest.mark.parametrize("Cout,Cin", WZ)
def test_winograd_image(hc, Cout, Cin, precision):
    got = hc.pack(weights(Cout, Cin, 3).cuda(), precision).cpu()
    assert torch.equal(got, reference(Cout, Cin, 3, precision))
    if precision != 6:
        check_scales(got, Cout, Cin, 36)


def test_phase_image(hc):
    import guided_diffusion._hip as H
    lib = H.load()
    Cout, Cin = 128, 16
    w = weights(Cout, Cin, 3).cuda()
    got = torch.empty(lib.ddpm3d_packed_up_phase_bytes(Cout, Cin), dtype=torch.uint8, device=w.device)
    H.check(lib.ddpm3d_pack_up_phase_weight(H.ptr(w), Cout, Cin, H.ptr(got), H.stream()))
    torch.cuda.synchronize()
    got = got.cpu()
    front, phase = R.up_phase_image(weights(Cout, Cin, 3))
    assert got.numel() == front.numel() + phase.numel()
    # the front is the precision-3 image of the same weights: the device's own, and the reference's
    assert torch.equal(got[:front.numel()], hc.pack(w, 3).cpu())
    assert torch.equal(got[:front.numel()], front)
    # the 64 phase taps and their scales
    assert torch.equal(got[front.numel():], phase)
    check_scales(got[front.numel():], Cout, Cin, 64)
